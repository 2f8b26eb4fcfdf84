"""Helpers of tests/test_spatial_userfunc_host.py and tests/test_gpu_spatial_userfunc.py: the reference's point
order restated with numpy, batches built from it, and plain-Python versions of the reference's three example
user functions (tilingstats.py:1037-1216)."""
import numpy as np


def visit_points(seg, band, null_val, tile, max_seg_id=None):
    """Every point (label in 1..max_seg_id, value != null_val) stably sorted by id in the reference's visit order
    (tile x tile tiles row-major, pixels row-major inside a tile): (ids, x, y, val)."""
    seg = np.asarray(seg)
    if max_seg_id is None:
        max_seg_id = int(seg.max()) if seg.size else 0
    (nr, nc) = seg.shape
    (r, c) = np.indices((nr, nc), dtype=np.int64)
    ntc = -(-nc // tile)
    rank = (((r // tile) * ntc + c // tile) * tile + r % tile) * tile + c % tile
    valid = (seg != 0) & (seg <= max_seg_id)
    if null_val is not None:
        valid &= band.astype(np.int64) != int(null_val)
    ids = seg[valid].astype(np.int64)
    order = np.lexsort((rank[valid], ids))
    return ids[order], c[valid][order], r[valid][order], band[valid].astype(np.int64)[order]


def as_points(x, y, val):
    pts = np.empty(len(x), dtype=[('x', np.uint32), ('y', np.uint32), ('val', np.int64)])
    (pts['x'], pts['y'], pts['val']) = (x, y, val)
    return pts.view(np.recarray)


def numpy_batches(seg, band, null_val, tile, ranges, max_seg_id=None):
    """(ids, offsets, pts) batches of the given id ranges, as iterSegmentPoints yields them."""
    (ids, x, y, val) = visit_points(seg, band, null_val, tile, max_seg_id)
    pts = as_points(x, y, val)
    pts.flags.writeable = False
    for (lo, hi) in ranges:
        bid = np.arange(lo, hi, dtype=np.uint32)
        cuts = np.searchsorted(ids, np.arange(lo, hi + 1))
        yield bid, (cuts - cuts[0]).astype(np.int64), pts[cuts[0]:cuts[-1]]


def mean_coord(pts, imgNullVal, intArr, floatArr, transform):
    """userFuncMeanCoord (tilingstats.py:1098-1142), point by point."""
    count = 0
    sumx = 0.0
    sumy = 0.0
    for pt in pts:
        geox = transform[0] + transform[1] * pt.x + transform[2] * pt.y
        geoy = transform[3] + transform[4] * pt.x + transform[5] * pt.y
        sumx += geox
        sumy += geoy
        count += 1
    floatArr[0] = sumx / count
    floatArr[1] = sumy / count


def mean_coord_vec(pts, imgNullVal, intArr, floatArr, transform):
    """mean_coord with numpy: the same products, summed strictly left to right (add.accumulate)."""
    (x, y) = (pts.x.astype(np.float64), pts.y.astype(np.float64))
    geox = transform[0] + transform[1] * x + transform[2] * y
    geoy = transform[3] + transform[4] * x + transform[5] * y
    floatArr[0] = np.add.accumulate(geox)[-1] / len(pts)
    floatArr[1] = np.add.accumulate(geoy)[-1] / len(pts)


def num_edge_pixels(pts, imgNullVal, intArr, floatArr, fourConnected):
    """userFuncNumEdgePixels (tilingstats.py:1146-1216)."""
    from pyshepseg_amd.tilingstats import convertPtsInto2DMaskArray
    mask = convertPtsInto2DMaskArray(pts, imgNullVal)
    outmask = mask.copy()
    (ysize, xsize) = mask.shape
    for y in range(ysize):
        for x in range(xsize):
            if mask[y, x] != 1:
                continue
            if y == 0 or x == 0 or y == ysize - 1 or x == xsize - 1:
                outmask[y, x] = 1
            elif fourConnected:
                total = int(mask[y - 1, x]) + mask[y + 1, x] + mask[y, x - 1] + mask[y, x + 1]
                outmask[y, x] = 0 if total == 4 else 1
            else:
                total = (int(mask[y - 1, x - 1]) + mask[y - 1, x] + mask[y + 1, x + 1] + mask[y, x - 1] +
                         mask[y, x + 1] + mask[y + 1, x - 1] + mask[y + 1, x] + mask[y + 1, x + 1])
                outmask[y, x] = 0 if total == 8 else 1
    intArr[0] = outmask.sum()


def variogram(pts, imgNullVal, intArr, floatArr, maxDist):
    """userFuncVariogram (tilingstats.py:1037-1094)."""
    from pyshepseg_amd.tilingstats import convertPtsInto2DArray
    tile = convertPtsInto2DArray(pts, imgNullVal)
    counts = np.zeros(maxDist, dtype=np.uint32)
    sumDifSqs = np.zeros(maxDist, dtype=np.float64)
    (ysize, xsize) = tile.shape
    for y in range(ysize):
        for x in range(xsize):
            val = int(tile[y, x])
            if val == imgNullVal:
                continue
            for yoffset in range(1, maxDist + 1):
                for xoffset in range(1, maxDist + 1):
                    if y + yoffset < ysize and x + xoffset < xsize:
                        val2 = int(tile[y + yoffset, x + xoffset])
                        if val2 == imgNullVal:
                            continue
                        dist = int(np.sqrt(yoffset * yoffset + xoffset * xoffset))
                        if 0 < dist <= maxDist:
                            counts[dist - 1] += 1
                            sumDifSqs[dist - 1] += (val - val2) ** 2
    for n in range(maxDist):
        if counts[n] > 0:
            floatArr[n] = np.sqrt(sumDifSqs[n] / counts[n])
