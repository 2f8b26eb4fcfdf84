"""The definition of segment hulls as a sequential model, and the hand-built rings the tests put through it.

With x = col and y = row the hull of an id is the strict convex hull of all vertices of its rings (Andrew's monotone
chain in Python integers: sort by (col, row), lower chain ascending, upper chain descending, a point popped while the
turn is not strictly to the left), which comes out oriented like an outer ring (positive under ringArea2's formula),
rotated to start at the hull vertex of the smallest (row, col).  hullReach of the edge from point k to its successor is
the largest |e x (q - p_k)| over the hull's points q and feretMax2 the largest squared distance of two hull points, both
by brute force over all pairs.  The float columns use math.fsum, math.sqrt and math.hypot."""
import itertools
import math

import numpy as np

import outline_cases as oc

SUMS = ('numHullVertices', 'hullArea2', 'feretMax2')
DERIVED = ('hullArea', 'solidity', 'hullPerimeter', 'convexity', 'feretMax', 'feretMin', 'feretRatio')


def cross(o, a, b):
    """(x, y) tuples"""
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def hull_of(points):
    """points: (row, col) pairs; the strict hull as (row, col) pairs in the stated order and from the stated start"""
    pts = sorted(set((int(c), int(r)) for (r, c) in points))
    if len(pts) > 1:
        chains = []
        for seq in (pts, pts[::-1]):
            ch = []
            for p in seq:
                while len(ch) >= 2 and cross(ch[-2], ch[-1], p) <= 0:
                    ch.pop()
                ch.append(p)
            chains.append(ch)
        pts = chains[0][:-1] + chains[1][:-1]
    k = min(range(len(pts)), key=lambda j: (pts[j][1], pts[j][0])) if pts else 0
    pts = pts[k:] + pts[:k]
    return [(y, x) for (x, y) in pts]


def extreme_points(points):
    """the strict extreme points by definition, all pairs and triples tried: p is none when it lies on the segment
    between two other points of the set, or in a proper triangle of three others (its rim included); a set of (row,
    col)"""
    pts = sorted(set((int(c), int(r)) for (r, c) in points))
    out = set()
    for p in pts:
        others = [q for q in pts if q != p]
        between = any(cross(a, b, p) == 0 and min(a[0], b[0]) <= p[0] <= max(a[0], b[0]) and
                      min(a[1], b[1]) <= p[1] <= max(a[1], b[1]) for (a, b) in itertools.combinations(others, 2))

        def holds(a, b, c):
            d = (cross(a, b, p), cross(b, c, p), cross(c, a, p))
            return cross(a, b, c) != 0 and (min(d) >= 0 or max(d) <= 0)
        if not between and not any(holds(*t) for t in itertools.combinations(others, 3)):
            out.add((p[1], p[0]))
    return out


def hull_numbers(h):
    """(reach per edge, area2, feretMax2) of a hull given as (row, col) pairs, by brute force"""
    n = len(h)
    if n == 0:
        return ([], 0, 0)
    p = np.array(h, dtype=np.int64)
    p = p - p.min(axis=0)
    assert p.max() < 2 ** 31 and int(p[:, 0].max()) * int(p[:, 1].max()) <= 2 ** 32
    (y, x) = (p[:, 0], p[:, 1])
    (ex, ey) = (np.roll(x, -1) - x, np.roll(y, -1) - y)
    # cross of edge k with (q - p_k), for all k and q
    cr = ex[:, None] * (y[None, :] - y[:, None]) - ey[:, None] * (x[None, :] - x[:, None])
    reach = np.abs(cr).max(axis=1)
    d2 = (x[:, None] - x[None, :]) ** 2 + (y[:, None] - y[None, :]) ** 2
    return ([int(v) for v in reach], oc.area2(p), int(d2.max()))


def reference_hulls(o, missing=-9999):
    """o: anything with maxSegId, ringOffsets, vertexOffsets, vertices, ringArea2.  A dictionary of hullOffsets,
    hullPoints, hullReach (int64), sums and columns"""
    S = int(o.maxSegId)
    (ro, vo, v, a2) = (np.asarray(o.ringOffsets), np.asarray(o.vertexOffsets), np.asarray(o.vertices), np.asarray(o.ringArea2))
    lengths = []
    for r in range(len(a2)):
        ring = v[vo[r]:vo[r + 1]]
        lengths.append(math.fsum(math.hypot(dr, dc) for (dr, dc) in (np.roll(ring, -1, axis=0) - ring).tolist()))
    hulls = []
    sums = {k: np.zeros(S + 1, dtype=np.int64) for k in SUMS}
    cols = {k: np.full(S + 1, float(missing), dtype=np.float64) for k in DERIVED}
    reach = []
    counts = np.zeros(S + 1, dtype=np.int64)
    for i in np.flatnonzero(np.diff(ro) > 0).tolist():          # (ids without rings: millions in the sparse rasters)
        rings = range(int(ro[i]), int(ro[i + 1]))
        h = hull_of(v[vo[ro[i]]:vo[ro[i + 1]]].tolist())
        hulls.append(h)
        if not h:
            continue
        counts[i] = len(h)
        (rch, area2, f2) = hull_numbers(h)
        reach.extend(rch)
        sums['numHullVertices'][i] = len(h)
        sums['hullArea2'][i] = area2
        sums['feretMax2'][i] = f2
        edges = [math.hypot(h[(j + 1) % len(h)][0] - h[j][0], h[(j + 1) % len(h)][1] - h[j][1]) for j in range(len(h))]
        per = math.fsum(lengths[r] for r in rings)
        cols['hullArea'][i] = area2 / 2.0
        cols['hullPerimeter'][i] = math.fsum(edges)
        cols['feretMax'][i] = math.sqrt(f2)
        cols['feretMin'][i] = min((rch[j] / edges[j] if edges[j] else 0.0) for j in range(len(h)))
        if area2:
            cols['solidity'][i] = sum(int(a2[r]) for r in rings) / area2
        if per:
            cols['convexity'][i] = cols['hullPerimeter'][i] / per
        if f2:
            cols['feretRatio'][i] = cols['feretMin'][i] / cols['feretMax'][i]
    columns = dict(sums)
    columns.update(cols)
    return dict(hullOffsets=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
                hullPoints=np.array([p for h in hulls for p in h], dtype=np.int64).reshape(-1, 2),
                hullReach=np.array(reach, dtype=np.int64), sums=sums, columns=columns, maxSegId=S)


# ---- hand-built rings -------------------------------------------------------------------------------------------------
def outlines_from_rings(rings, maxSegId=None, origin=(0, 0)):
    """rings: {id: [ring, ...]}, a ring a list of (row, col) without the origin; a SegmentOutlines as a trace would
    leave it (ringArea2 from the vertices: give outer rings clockwise on screen)"""
    from pyshepseg_amd import outlines
    if maxSegId is None:
        maxSegId = max(rings) if rings else 0
    (counts, vcounts, verts, area2) = (np.zeros(maxSegId + 1, dtype=np.int64), [], [], [])
    for i in sorted(rings):
        for ring in rings[i]:
            counts[i] += 1
            vcounts.append(len(ring))
            verts.extend(ring)
            area2.append(oc.area2(ring))
    v = np.array(verts, dtype=np.int64).reshape(-1, 2) + np.array(origin, dtype=np.int64)
    return outlines.SegmentOutlines(maxSegId, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
                                    np.concatenate([[0], np.cumsum(vcounts)]).astype(np.int64), v,
                                    np.array(area2, dtype=np.int64), origin=tuple(origin))


def histogram_ring(heights, base=None):
    """the rectilinear outer ring of a histogram: column c covers the cols [c, c + 1] and the rows [base - heights[c],
    base] (heights >= 1; base defaults to the largest height, so the highest top is row 0)"""
    heights = [int(h) for h in heights]
    assert heights and min(heights) >= 1
    if base is None:
        base = max(heights)
    ring = []
    for (c, h) in enumerate(heights):
        if c == 0 or heights[c - 1] != h:
            ring.append((base - h, c))
        if c + 1 == len(heights) or heights[c + 1] != h:
            ring.append((base - h, c + 1))
    ring += [(base, len(heights)), (base, 0)]
    assert oc.area2(ring) == 2 * sum(heights)
    return ring


def mirrored(ring, rows=False, cols=False, extent=None):
    """the ring mirrored in the rows and / or columns 0 .. extent (default: its own largest), its sense of rotation kept"""
    r = np.array(ring, dtype=np.int64)
    if extent is None:
        extent = r.max(axis=0)
    if rows:
        r[:, 0] = extent[0] - r[:, 0]
    if cols:
        r[:, 1] = extent[1] - r[:, 1]
    out = [tuple(p) for p in r.tolist()]
    return out[::-1] if rows != cols else out


def cascade_heights(n, flat=False):
    """tops K - (n - c)^2 for c = 0 .. n, every one a hull vertex of the columns before the last, and a final column
    above every tangent line of them: the upper chain of the whole is two points, found by popping all the others.
    flat: the first two columns level, which takes one vertex out (an odd number of kept points)"""
    K = n * n + 1
    h = [K - (n - c) ** 2 for c in range(n + 1)]
    if flat:
        h[0] = h[1]
    return h + [K + 2 * n * n + 10]


def rectangle_ring(r0, c0, a, b):
    return [(r0, c0), (r0, c0 + b), (r0 + a, c0 + b), (r0 + a, c0)]


def diamond(radius):
    """the digital disc |y| + |x| <= radius as a label raster of id 1"""
    (y, x) = np.indices((2 * radius + 1, 2 * radius + 1)) - radius
    return (np.abs(y) + np.abs(x) <= radius).astype(np.uint32)


def parallelogram(n=200, width=3):
    """a long thin diagonal staircase: row y holds the pixels y .. y + width - 1"""
    seg = np.zeros((n, n + width), dtype=np.uint32)
    for y in range(n):
        seg[y, y:y + width] = 1
    return seg


L_SHAPE = np.array([[1, 0, 0], [1, 0, 0], [1, 1, 1]], dtype=np.uint32)
PLUS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=np.uint32)
RING = np.array([[1, 1, 1, 1], [1, 0, 0, 1], [1, 0, 2, 1], [1, 1, 1, 1]], dtype=np.uint32)


def end_pixels(rows=64, width=4097):
    """id i = the first and the last pixel of row i - 1"""
    seg = np.zeros((rows, width), dtype=np.uint32)
    seg[:, 0] = seg[:, -1] = np.arange(1, rows + 1, dtype=np.uint32)
    return seg
