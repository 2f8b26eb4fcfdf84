"""The definition of the junction trace and of the topology-aware Douglas-Peucker simplification as a sequential model
in Python integers, and the rings the tests put through it.

Junction.  Labels outside the raster read as 0.  The four pixels round a corner are a b / c d; the corner's degree is the
number of the pairs (a, b), (b, d), (c, d), (a, c) whose labels differ (0, 2, 3 or 4); a corner of degree >= 3 is a
junction, whatever the corner rule of the trace.

Junction trace.  outline_cases' walk, with a vertex at every edge that is a turn edge or whose start corner is a
junction; a ring starts at its vertex edge of the smallest key, rings are ordered by (id, that key).

Simplification.  A ring's anchors are its flagged vertices; a ring without any takes its vertex of the smallest (row,
col) (the first of equal ones).  An arc runs from one anchor to the next in ring order, cyclically, both included.  Both
ends of an arc are kept.  Between kept a and b: m(q) = |(b - a) x (q - a)| if a != b, |q - a|^2 if a = b; the candidate is
the point of the largest m, ties to the smallest (row, col), then to the first in arc order; it exceeds when
m^2 65536 > T |b - a|^2 (a != b) or m 65536 > T (a = b), T = floor(tolerance^2 65536); if it exceeds it is kept and both
halves are treated the same way.  A ring is dropped when fewer than three vertices remain or when its new ringArea2 is 0
or differs in sign from its source ring's."""
import math

import numpy as np

import outline_cases as oc

TOLERANCES = (0.0, 0.5, 1.0, 1.5, 4.0)
# points of an arc up to which one wavefront / one workgroup takes it (csrc/simplify.h: SP_SHORT_MAX, SP_GROUP_MAX)
SHORT_MAX = 64
GROUP_MAX = 1024


def tolerance2q(tolerance):
    return int(math.floor(float(tolerance) * float(tolerance) * 65536.0))


# ---- the junction trace -------------------------------------------------------------------------------------------------
def corner_degrees(seg):
    """degree of every corner (row, col), 0 <= row <= H, 0 <= col <= W"""
    p = np.pad(np.asarray(seg), 1)
    (a, b, c, d) = (p[:-1, :-1], p[:-1, 1:], p[1:, :-1], p[1:, 1:])
    return (a != b).astype(np.int64) + (b != d) + (c != d) + (a != c)


def walk_junction_rings(seg, fourConnected=True):
    """every ring as (id, key of its first vertex edge, [vertices], [junction flags])"""
    seg = np.asarray(seg)
    lab = np.pad(seg, 1).tolist()
    deg = corner_degrees(seg).tolist() if seg.size else []
    p = np.pad(seg, 1)
    across = [p[:-2, 1:-1], p[1:-1, 2:], p[2:, 1:-1], p[1:-1, :-2]]
    isedge = np.stack([(seg != 0) & (o != seg) for o in across], axis=-1)
    seen = set()
    rings = []
    for (y0, x0, s0) in np.argwhere(isedge).tolist():
        if (y0, x0, s0) in seen:
            continue
        a = lab[y0 + 1][x0 + 1]
        (y, x, s) = (y0, x0, s0)
        cycle = []
        while (y, x, s) not in seen:
            seen.add((y, x, s))
            cycle.append((y, x, s))
            (dy, dx) = oc.DIRS[s]
            (ay, ax) = oc.DIRS[(s + 3) & 3]
            right = lab[y + dy + 1][x + dx + 1] == a
            left = lab[y + dy + ay + 1][x + dx + ax + 1] == a
            if right and not left:
                (y, x) = (y + dy, x + dx)
            elif left and (right or not fourConnected):
                (y, x, s) = (y + dy + ay, x + dx + ax, (s + 3) & 3)
            else:
                s = (s + 1) & 3
        assert (y, x, s) == (y0, x0, s0)

        def start(e):
            return (e[0] + oc.START[e[2]][0], e[1] + oc.START[e[2]][1])
        vs = [e for (i, e) in enumerate(cycle) if cycle[i - 1][2] != e[2] or deg[start(e)[0]][start(e)[1]] >= 3]
        k = vs.index(min(vs))
        vs = vs[k:] + vs[:k]
        rings.append((a, vs[0], [start(e) for e in vs], [1 if deg[start(e)[0]][start(e)[1]] >= 3 else 0 for e in vs]))
    return rings


def pack_rings(rings, maxSegId, origin=(0, 0)):
    """rings: (id, sort key, [vertices], [flags]) -> the arrays of a SegmentOutlines and ``junction``"""
    rings = sorted(rings, key=lambda r: (r[0], r[1]))
    counts = np.bincount(np.array([r[0] for r in rings], dtype=np.int64), minlength=maxSegId + 1)
    verts = np.array([v for r in rings for v in r[2]], dtype=np.int64).reshape(-1, 2) + np.array(origin, dtype=np.int64)
    return dict(ringOffsets=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
                vertexOffsets=np.concatenate([[0], np.cumsum([len(r[2]) for r in rings])]).astype(np.int64), vertices=verts,
                ringArea2=np.array([oc.area2(r[2]) for r in rings], dtype=np.int64),
                junction=np.array([f for r in rings for f in r[3]], dtype=np.uint8), maxSegId=maxSegId)


def reference_junction_trace(seg, fourConnected=True, maxSegId=None, origin=(0, 0)):
    seg = np.asarray(seg)
    if maxSegId is None:
        maxSegId = int(seg.max()) if seg.size else 0
    return pack_rings(walk_junction_rings(seg, fourConnected), maxSegId, origin)


# ---- the simplification ---------------------------------------------------------------------------------------------------
def measure(a, b, q):
    if a == b:
        return (q[0] - a[0]) ** 2 + (q[1] - a[1]) ** 2
    return abs((b[0] - a[0]) * (q[1] - a[1]) - (b[1] - a[1]) * (q[0] - a[0]))


def exceeds(m, a, b, T):
    if a == b:
        return m * 65536 > T
    return m * m * 65536 > T * ((b[0] - a[0]) ** 2 + (b[1] - a[1]) ** 2)


def simplify_arc(pts, T):
    """(kept flag per point, depth of the recursion) of an arc of (row, col) tuples of Python integers"""
    n = len(pts)
    kept = [False] * n
    kept[0] = kept[n - 1] = True
    if n == 2:
        return (kept, 0)
    depth = 0
    stack = [(0, n - 1, 1)]
    while stack:
        (lo, hi, level) = stack.pop()
        if hi - lo < 2:
            continue
        (a, b) = (pts[lo], pts[hi])
        best = min(range(lo + 1, hi), key=lambda i: (-measure(a, b, pts[i]), pts[i], i))
        if exceeds(measure(a, b, pts[best]), a, b, T):
            kept[best] = True
            depth = max(depth, level)
            stack.append((lo, best, level + 1))
            stack.append((best, hi, level + 1))
    return (kept, depth)


def ring_arcs(pts, flags):
    """the arcs of a ring as lists of positions in the ring, ends included"""
    n = len(pts)
    anchors = [i for i in range(n) if flags[i]]
    if not anchors:
        anchors = [min(range(n), key=lambda i: (pts[i], i))]
    arcs = []
    for (t, s) in enumerate(anchors):
        steps = (anchors[(t + 1) % len(anchors)] - s) % n or n
        arcs.append([(s + q) % n for q in range(steps + 1)])
    return arcs


def sign(v):
    return (v > 0) - (v < 0)


def ring_area2(pts):
    """sum(c_i r_(i+1) - c_(i+1) r_i) in Python integers"""
    return sum(pts[i][1] * pts[(i + 1) % len(pts)][0] - pts[(i + 1) % len(pts)][1] * pts[i][0] for i in range(len(pts)))


def reference_simplify(o, tolerance=None, T=None):
    """o: anything with ringOffsets, vertexOffsets, vertices, ringArea2, junction (attributes or keys).  A dictionary of
    the int64 arrays of a SimplifiedOutlines, ``kept`` (a flag per source vertex), ``rounds``, ``arcs``, ``longestArc``"""
    get = (lambda k: o[k]) if isinstance(o, dict) else (lambda k: getattr(o, k))
    if T is None:
        T = tolerance2q(tolerance)
    (ro, vo, a2) = (np.asarray(get('ringOffsets')), np.asarray(get('vertexOffsets')), np.asarray(get('ringArea2')))
    v = np.asarray(get('vertices')).tolist()
    flags = np.asarray(get('junction')).tolist()
    kept = np.zeros(len(v), dtype=bool)
    (rounds, narcs, longest) = (0, 0, 0)
    for k in range(len(a2)):
        (b, e) = (int(vo[k]), int(vo[k + 1]))
        if e == b:
            continue
        pts = [tuple(p) for p in v[b:e]]
        for arc in ring_arcs(pts, flags[b:e]):
            (flag, depth) = simplify_arc([pts[i] for i in arc], T)
            for (i, f) in zip(arc, flag):
                if f:
                    kept[b + i] = True
            (rounds, narcs, longest) = (max(rounds, depth), narcs + 1, max(longest, len(arc)))
    (sourceRing, keptVertex, area, offs) = ([], [], [], [0])
    for k in range(len(a2)):
        idx = [i for i in range(int(vo[k]), int(vo[k + 1])) if kept[i]]
        now = ring_area2([v[i] for i in idx])
        if len(idx) < 3 or now == 0 or sign(now) != sign(int(a2[k])):
            continue
        sourceRing.append(k)
        keptVertex += idx
        area.append(now)
        offs.append(len(keptVertex))
    sourceRing = np.array(sourceRing, dtype=np.int64)
    alive = np.zeros(len(a2) + 1, dtype=np.int64)
    alive[1:][sourceRing] = 1
    ringOffsets = np.cumsum(alive)[ro].astype(np.int64)
    keptVertex = np.array(keptVertex, dtype=np.int64)
    return dict(ringOffsets=ringOffsets, vertexOffsets=np.array(offs, dtype=np.int64),
                vertices=np.asarray(get('vertices'))[keptVertex].reshape(-1, 2).astype(np.int64),
                ringArea2=np.array(area, dtype=np.int64), sourceRing=sourceRing, keptVertex=keptVertex,
                droppedRings=(np.diff(ro) - np.diff(ringOffsets)).astype(np.int64), kept=kept, rounds=rounds, arcs=narcs,
                longestArc=longest, junction=np.asarray(get('junction'))[keptVertex])


def corner_flags(vertices, kept):
    """{corner: set of the kept flags of the vertices at it}"""
    out = {}
    for (p, f) in zip(np.asarray(vertices).tolist(), np.asarray(kept).tolist()):
        out.setdefault(tuple(p), set()).add(bool(f))
    return out


# ---- rings built by hand ----------------------------------------------------------------------------------------------
def arc_ring(points, wrap=0, far=None):
    """A ring (vertices, flags) whose first arc is ``points`` between two flagged ends; it closes through one more
    flagged vertex far below, so its other two arcs have two points each.  ``wrap`` rotates the vertex list so that
    the arc begins ``wrap`` places before the list's end and wraps round it."""
    pts = [tuple(int(x) for x in p) for p in points]
    if far is None:
        far = (max(p[0] for p in pts) + 1000, min(p[1] for p in pts) - 7)
    verts = pts + [far]
    flags = [1] + [0] * (len(pts) - 2) + [1, 1]
    if wrap:
        k = len(verts) - wrap
        (verts, flags) = (verts[-k:] + verts[:-k], flags[-k:] + flags[:-k]) if k else (verts, flags)
    return (verts, flags)


def outlines_from(rings, maxSegId=None):
    """rings: {id: [(vertices, flags), ...]} -> the arrays of a SegmentOutlines and ``junction``"""
    if maxSegId is None:
        maxSegId = max(rings)
    return pack_rings([(i, n, r[0], r[1]) for i in rings for (n, r) in enumerate(rings[i])], maxSegId)


def zigzag(n):
    """(k, (-1)^k k), k = 0 .. n - 1: at tolerance 0.5 the recursion keeps one point per level, from the far end down"""
    pts = [(k, k if k % 2 == 0 else -k) for k in range(n)]
    (kept, depth) = simplify_arc(pts, tolerance2q(0.5))
    assert depth >= n / 2, (n, depth)
    return pts


def wobble(n, seed=0):
    """an arc of n distinct points that advances a row per point and wanders in the columns"""
    rng = np.random.default_rng(1000 * n + seed)
    return [(k, int(c)) for (k, c) in enumerate(np.cumsum(rng.integers(-3, 4, size=n)))]


def many_arcs(narcs):
    """one ring of ``narcs`` arcs of three points each: the flagged vertices (0, 2 i) along the top with (1, 2 i + 1)
    between them, and the way back far below"""
    n = narcs - 1
    verts = []
    flags = []
    for i in range(n):
        verts += [(0, 2 * i), (1 + i % 3, 2 * i + 1)]
        flags += [1, 0]
    verts += [(0, 2 * n), (50, n)]
    flags += [1, 0]
    return (verts, flags)


TIE_ARC = [(0, 0), (3, 2), (0, 4), (3, 6), (0, 8)]
