"""The definition of the per-segment shape table in numpy, and the label rasters the tests put through it beyond those
of tests/neighbour_cases.py.

With (r, c) = (row0 + y, col0 + x) the coordinates of pixel (y, x) and label 0 no segment, per id: ``area``; the extent
``rowMin`` .. ``colMax``; ``perimeter``, the N, S, W, E sides of the id's pixels whose other side is a different label,
label 0 or outside the raster; ``outerBorder``, those whose other side is label 0 or outside; ``edgePixels``, pixels
with at least one such side; and the sums of r, c, r^2, c^2, r c modulo 2^64.  Ids without pixels hold 0 everywhere."""
import numpy as np

from neighbour_cases import (EXAMPLE, OFF_GRID_SHAPES, PATCH_COLS, PATCH_ROWS, SPARSE_MAX, WIDE_MAX,  # noqa: F401
                             enclosed_by_zeros, every_pixel_its_own, half_planes, hot_segment, random_labels,
                             sparse_ids, stripes, wide_ids)

COUNTS = ('area', 'rowMin', 'rowMax', 'colMin', 'colMax', 'perimeter', 'outerBorder', 'edgePixels')
SUMS = ('sumRow', 'sumCol', 'sumRowRow', 'sumColCol', 'sumRowCol')
MASK64 = (1 << 64) - 1

# the worked example, EXAMPLE = [[1, 1, 2], [1, 3, 2], [0, 3, 3]], rows 0 .. 3 written out by hand
EXAMPLE_COUNTS = {'area': [0, 3, 2, 3], 'rowMin': [0, 0, 0, 1], 'rowMax': [0, 1, 1, 2], 'colMin': [0, 0, 2, 1],
                  'colMax': [0, 1, 2, 2], 'perimeter': [0, 8, 6, 8], 'outerBorder': [0, 5, 3, 4],
                  'edgePixels': [0, 3, 2, 3]}
EXAMPLE_SUMS = {'sumRow': [0, 1, 1, 5], 'sumCol': [0, 1, 4, 4], 'sumRowRow': [0, 1, 1, 9], 'sumColCol': [0, 1, 8, 6],
                'sumRowCol': [0, 0, 2, 7]}


def _sides(seg):
    """(differs, outer): bool [4, rows, cols] for N, S, W, E -- the side's other label differs from the pixel's (or
    lies outside the raster), the side's other label is 0 (or lies outside); both False where the pixel is 0"""
    p = np.pad(seg, 1)
    others = [p[:-2, 1:-1], p[2:, 1:-1], p[1:-1, :-2], p[1:-1, 2:]]
    own = seg != 0
    return (np.stack([own & (o != seg) for o in others]), np.stack([own & (o == 0) for o in others]))


def reference_shapes(seg, maxSegId=None, origin=(0, 0)):
    """(counts, sums): dictionaries of int64 COUNTS and uint64 SUMS, maxSegId + 1 rows each; the sums wrap modulo 2^64
    as numpy's uint64 arithmetic does"""
    seg = np.asarray(seg)
    assert seg.ndim == 2 and seg.dtype == np.uint32
    if maxSegId is None:
        maxSegId = int(seg.max()) if seg.size else 0
    n = maxSegId + 1
    (differs, outer) = _sides(seg)
    (ys, xs) = np.nonzero(seg)
    lab = seg[ys, xs].astype(np.int64)
    counts = {'area': np.bincount(lab, minlength=n).astype(np.int64),
              'perimeter': np.bincount(lab, weights=differs.sum(axis=0)[ys, xs], minlength=n).astype(np.int64),
              'outerBorder': np.bincount(lab, weights=outer.sum(axis=0)[ys, xs], minlength=n).astype(np.int64),
              'edgePixels': np.bincount(lab, weights=differs.any(axis=0)[ys, xs], minlength=n).astype(np.int64)}
    r = ys.astype(np.int64) + int(origin[0])
    c = xs.astype(np.int64) + int(origin[1])
    big = np.iinfo(np.int64).max
    for (name, v, at, init) in (('rowMin', r, np.minimum.at, big), ('rowMax', r, np.maximum.at, -1),
                                ('colMin', c, np.minimum.at, big), ('colMax', c, np.maximum.at, -1)):
        col = np.full(n, init, dtype=np.int64)
        at(col, lab, v)
        col[counts['area'] == 0] = 0
        counts[name] = col
    (ru, cu) = (r.astype(np.uint64), c.astype(np.uint64))
    sums = {}
    for (name, v) in (('sumRow', ru), ('sumCol', cu), ('sumRowRow', ru * ru), ('sumColCol', cu * cu),
                      ('sumRowCol', ru * cu)):
        col = np.zeros(n, dtype=np.uint64)
        np.add.at(col, lab, v)
        sums[name] = col
    return ({k: counts[k] for k in COUNTS}, sums)


def reference_shapes_pyint(seg, maxSegId=None, origin=(0, 0)):
    """reference_shapes in Python integers, pixel by pixel: nothing wraps before the final ``& MASK64``, so origins
    near 2^32 (where r^2 and r c pass 2^63) are checked independently of numpy's modular arithmetic"""
    seg = np.asarray(seg)
    (nrows, ncols) = seg.shape
    if maxSegId is None:
        maxSegId = int(seg.max()) if seg.size else 0
    n = maxSegId + 1
    counts = {k: [0] * n for k in COUNTS}
    sums = {k: [0] * n for k in SUMS}
    cells = seg.tolist()

    def at(y, x):
        return cells[y][x] if 0 <= y < nrows and 0 <= x < ncols else 0
    for y in range(nrows):
        for x in range(ncols):
            v = cells[y][x]
            if v == 0:
                continue
            (r, c) = (int(origin[0]) + y, int(origin[1]) + x)
            others = [at(y - 1, x), at(y + 1, x), at(y, x - 1), at(y, x + 1)]
            if counts['area'][v] == 0:
                (counts['rowMin'][v], counts['rowMax'][v], counts['colMin'][v], counts['colMax'][v]) = (r, r, c, c)
            counts['area'][v] += 1
            counts['rowMin'][v] = min(counts['rowMin'][v], r)
            counts['rowMax'][v] = max(counts['rowMax'][v], r)
            counts['colMin'][v] = min(counts['colMin'][v], c)
            counts['colMax'][v] = max(counts['colMax'][v], c)
            counts['perimeter'][v] += sum(o != v for o in others)
            counts['outerBorder'][v] += sum(o == 0 for o in others)
            counts['edgePixels'][v] += int(any(o != v for o in others))
            for (name, t) in (('sumRow', r), ('sumCol', c), ('sumRowRow', r * r), ('sumColCol', c * c), ('sumRowCol', r * c)):
                sums[name][v] += t
    return ({k: np.array(counts[k], dtype=np.int64) for k in COUNTS},
            {k: np.array([t & MASK64 for t in sums[k]], dtype=np.uint64) for k in SUMS})


def rectangle_sums(h, w, origin=(0, 0)):
    """(counts, sums) of rows 0 and 1 for one h x w rectangle of label 1 alone in the world, in Python integers"""
    return reference_shapes_pyint(np.ones((h, w), dtype=np.uint32), 1, origin)


# ---- rasters for the kernel's run aggregation and its LDS table ------------------------------------------------------
TABLE_SLOTS = 512           # SHAPE_SLOTS of csrc/segshape.h: a patch with more distinct labels takes the overflow route


def runs_end_on_lane_63():
    """every patch row holds a run that ends on the patch's last column and one that begins on the next patch's
    first: 3 patch columns, labels change at columns 50 and 64 of every 64"""
    x = np.arange(200, dtype=np.uint32)
    row = 1 + 2 * (x // 64) + (x % 64 >= 50)
    return np.ascontiguousarray(np.broadcast_to(row, (70, 200))).astype(np.uint32)


def label_home(label):
    """shape_hash of csrc/segshape.h: the slot of a patch's table where a label is looked for first"""
    label = np.asarray(label, dtype=np.uint64)
    return ((((label * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(16)) &
            np.uint64(TABLE_SLOTS - 1)).astype(np.int64)


def table_fill(distinct):
    """a 96 x 192 raster of 1s whose patch (1, 1) holds exactly ``distinct`` distinct labels: the background and
    ``distinct - 1`` pixels with labels of their own from 2, on every second column of its rows"""
    seg = np.ones((3 * PATCH_ROWS, 3 * PATCH_COLS), dtype=np.uint32)
    k = np.arange(distinct - 1)
    assert distinct - 1 <= PATCH_ROWS * (PATCH_COLS // 2)
    seg[PATCH_ROWS + k // (PATCH_COLS // 2), PATCH_COLS + 2 * (k % (PATCH_COLS // 2))] = 2 + k
    return seg


TABLE_WRAP_HOME = 5


def table_wrap():
    """a 96 x 192 raster of 0s whose patch (1, 1) holds exactly TABLE_SLOTS labels that all have the SAME home slot, in
    blocks of 2 x 2 pixels: linear probing puts them in 512 slots in a row, and whichever arrives last finds its slot
    with the last probe of its trip round the table"""
    cand = np.arange(1, 1 << 20, dtype=np.int64)
    labels = cand[label_home(cand) == TABLE_WRAP_HOME][:TABLE_SLOTS]
    assert len(labels) == TABLE_SLOTS
    seg = np.zeros((3 * PATCH_ROWS, 3 * PATCH_COLS), dtype=np.uint32)
    grid = labels.reshape(PATCH_ROWS // 2, PATCH_COLS // 2).astype(np.uint32)
    seg[PATCH_ROWS:2 * PATCH_ROWS, PATCH_COLS:2 * PATCH_COLS] = np.repeat(np.repeat(grid, 2, axis=0), 2, axis=1)
    return seg


def tall_and_wide():
    """a 70000 x 3 and a 3 x 70000 raster of a few labels: r^2 and c^2 pass 2^32, their sums 2^47"""
    k = (np.arange(70000, dtype=np.uint32) // 9000) % 4
    tall = np.ascontiguousarray(np.stack([k, (k + 1) % 4, np.full(70000, 2, dtype=np.uint32)], axis=1)).astype(np.uint32)
    return (tall, np.ascontiguousarray(tall.T))
