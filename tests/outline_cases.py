"""The definition of segment outlines as a sequential model, and the label rasters the tests put through it.

Pixel (y, x) covers [y, y + 1] x [x, x + 1]; corners are integer (row, col) pairs; label 0 is no segment.  A side of a
pixel of id A is an edge of A when the label across it differs from A (another id, label 0, outside the raster: the
``perimeter`` of shapes.py).  Edges are directed with A's pixel on the right of travel:

    side 0 (N): (y, x) -> (y, x + 1)            side 2 (S): (y + 1, x + 1) -> (y + 1, x)
    side 1 (E): (y, x + 1) -> (y + 1, x + 1)    side 3 (W): (y + 1, x) -> (y, x)

and an edge's key is (y, x, side).  The successor of an edge is decided at its end corner by R (the pixel right-ahead
is A) and L (the pixel left-ahead is A): not R -> the next side of the same pixel; R and not L -> the same side of the
pixel right-ahead; R and L -> side - 1 of the pixel left-ahead; the saddle (not R, L) turns right when four-connected
and left when eight-connected.  A turn edge is an edge whose predecessor has another side number; a ring is a cycle of
the successor map, its vertices the start corners of its turn edges from the turn edge of the smallest key (the
leader) on; ringArea2 = sum(c_i r_{i+1} - c_{i+1} r_i); rings are ordered by (id, leader key).

The model finds the sides with numpy and walks every cycle edge by edge."""
import numpy as np

from neighbour_cases import SPARSE_MAX, WIDE_MAX, random_labels, sparse_ids, wide_ids  # noqa: F401

# direction of travel per side, as (dy, dx); the pixel across side s lies at DIRS[(s + 3) & 3]
DIRS = ((0, 1), (1, 0), (0, -1), (-1, 0))
# start corner of side s of pixel (0, 0)
START = ((0, 0), (0, 1), (1, 1), (1, 0))

COLUMNS = ('numParts', 'numHoles', 'numVertices', 'holeArea')

EXAMPLE = np.array([[1, 1, 2], [1, 2, 2], [3, 3, 2]], dtype=np.uint32)
EXAMPLE_RINGS = {1: [[(0, 0), (0, 2), (1, 2), (1, 1), (2, 1), (2, 0)]],
                 2: [[(0, 2), (0, 3), (3, 3), (3, 2), (2, 2), (2, 1), (1, 1), (1, 2)]],
                 3: [[(2, 0), (2, 2), (3, 2), (3, 0)]]}
EXAMPLE_AREA2 = [6, 8, 4]


def walk_rings(seg, fourConnected=True):
    """every ring of the raster as (id, leader key, [vertices], edges of the ring), in the order of the smallest edge"""
    seg = np.asarray(seg)
    (nrows, ncols) = seg.shape
    lab = np.pad(seg, 1).tolist()               # lab[y + 1][x + 1]
    p = np.pad(seg, 1)
    across = [p[:-2, 1:-1], p[1:-1, 2:], p[2:, 1:-1], p[1:-1, :-2]]        # N, E, S, W
    isedge = np.stack([(seg != 0) & (o != seg) for o in across], axis=-1)   # [y, x, side]
    seen = set()
    rings = []
    for (y0, x0, s0) in np.argwhere(isedge).tolist():      # in key order
        if (y0, x0, s0) in seen:
            continue
        a = lab[y0 + 1][x0 + 1]
        (y, x, s) = (y0, x0, s0)
        cycle = []
        while (y, x, s) not in seen:
            seen.add((y, x, s))
            cycle.append((y, x, s))
            (dy, dx) = DIRS[s]
            (ay, ax) = DIRS[(s + 3) & 3]
            right = lab[y + dy + 1][x + dx + 1] == a
            left = lab[y + dy + ay + 1][x + dx + ax + 1] == a
            if right and not left:
                (y, x) = (y + dy, x + dx)
            elif left and (right or not fourConnected):
                (y, x, s) = (y + dy + ay, x + dx + ax, (s + 3) & 3)
            else:
                s = (s + 1) & 3
        assert (y, x, s) == (y0, x0, s0), 'the successor map is no permutation'
        turns = [e for (i, e) in enumerate(cycle) if cycle[i - 1][2] != e[2]]
        lead = min(turns)
        k = turns.index(lead)
        turns = turns[k:] + turns[:k]
        rings.append((a, lead, [(e[0] + START[e[2]][0], e[1] + START[e[2]][1]) for e in turns], len(cycle)))
    assert sum(r[3] for r in rings) == int(isedge.sum())
    return rings


def area2(verts):
    v = np.asarray(verts, dtype=np.int64).reshape(-1, 2)
    (r, c) = (v[:, 0], v[:, 1])
    return int(np.sum(c * np.roll(r, -1) - np.roll(c, -1) * r))


def columns_from_rings(ringOffsets, vertexOffsets, ringArea2):
    """the per-id columns, ring by ring in Python"""
    n = len(ringOffsets) - 1
    cols = {k: np.zeros(n, dtype=np.int64) for k in COLUMNS}
    for i in range(n):
        for r in range(int(ringOffsets[i]), int(ringOffsets[i + 1])):
            cols['numVertices'][i] += int(vertexOffsets[r + 1] - vertexOffsets[r])
            if ringArea2[r] > 0:
                cols['numParts'][i] += 1
            else:
                cols['numHoles'][i] += 1
                cols['holeArea'][i] += -int(ringArea2[r]) // 2
    return cols


def reference_outlines(seg, fourConnected=True, maxSegId=None, origin=(0, 0)):
    """a dictionary of ringOffsets, vertexOffsets, vertices, ringArea2 (all int64), columns and ringEdges (the edges of
    every ring, int64)"""
    seg = np.asarray(seg)
    assert seg.ndim == 2 and seg.dtype == np.uint32
    if maxSegId is None:
        maxSegId = int(seg.max()) if seg.size else 0
    rings = sorted(walk_rings(seg, fourConnected), key=lambda r: (r[0], r[1]))
    assert all(r[0] <= maxSegId for r in rings)
    counts = np.bincount(np.array([r[0] for r in rings], dtype=np.int64), minlength=maxSegId + 1)
    ringOffsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    vertexOffsets = np.concatenate([[0], np.cumsum([len(r[2]) for r in rings])]).astype(np.int64)
    verts = np.array([v for r in rings for v in r[2]], dtype=np.int64).reshape(-1, 2)
    ringArea2 = np.array([area2(r[2]) for r in rings], dtype=np.int64)
    verts = verts + np.array(origin, dtype=np.int64)
    return dict(ringOffsets=ringOffsets, vertexOffsets=vertexOffsets, vertices=verts, ringArea2=ringArea2,
                columns=columns_from_rings(ringOffsets, vertexOffsets, ringArea2),
                ringEdges=np.array([r[3] for r in rings], dtype=np.int64), maxSegId=maxSegId)


def ring_lengths(vertexOffsets, vertices):
    """edges of every ring: the Manhattan length of its vertex sequence"""
    vo = np.asarray(vertexOffsets)
    v = np.asarray(vertices)
    if len(v) == 0:
        return np.zeros(len(vo) - 1, dtype=np.int64)
    nxt = np.arange(len(v)) + 1
    ringOf = np.repeat(np.arange(len(vo) - 1), np.diff(vo))
    last = nxt == vo[1:][ringOf]
    nxt[last] = vo[:-1][ringOf][last]
    step = np.abs(v[nxt] - v).sum(axis=1)
    cs = np.concatenate([[0], np.cumsum(step)])
    return (cs[vo[1:]] - cs[vo[:-1]]).astype(np.int64)


def rasterise(shape, ringOffsets, vertexOffsets, vertices, origin=(0, 0)):
    """the label raster back from the rings: a vertical ring segment from (r0, c) to (r1, c) takes the ring's id from
    cell (r0, c) and adds it to cell (r1, c) of a difference array; summing down the rows makes that -+ id over the
    segment's rows, and summing along the columns fills every id between its left and right sides"""
    ro = np.asarray(ringOffsets)
    vo = np.asarray(vertexOffsets)
    v = np.asarray(vertices) - np.array(origin, dtype=np.int64)
    d = np.zeros((shape[0] + 1, shape[1] + 1), dtype=np.int64)
    if len(v):
        idOfRing = np.repeat(np.arange(len(ro) - 1), np.diff(ro))
        ringOf = np.repeat(np.arange(len(vo) - 1), np.diff(vo))
        nxt = np.arange(len(v)) + 1
        last = nxt == vo[1:][ringOf]
        nxt[last] = vo[:-1][ringOf][last]
        vert = v[nxt][:, 1] == v[:, 1]
        ids = idOfRing[ringOf][vert]
        np.add.at(d, (v[vert, 0], v[vert, 1]), -ids)
        np.add.at(d, (v[nxt][vert, 0], v[vert, 1]), ids)
    return np.cumsum(np.cumsum(d, axis=0), axis=1)[:shape[0], :shape[1]]


# ---- rasters ----------------------------------------------------------------------------------------------------------
def checkerboard(n):
    (y, x) = np.indices((n, n))
    return ((y + x) % 2).astype(np.uint32)


def saddles():
    """two pixels of one id touching diagonally, in each corner of the raster and across each rim, both diagonals"""
    out = []
    for (h, w) in ((2, 2), (5, 7)):
        for (y, x) in {(0, 0), (0, w - 2), (h - 2, 0), (h - 2, w - 2), (0, w // 2 - 1), (h - 2, w // 2 - 1),
                       (h // 2 - 1, 0), (h // 2 - 1, w - 2)}:
            for (a, b) in ((1, 2), (1, 0)):
                for flip in (False, True):
                    seg = np.full((h, w), b, dtype=np.uint32)
                    if flip:
                        seg[y, x + 1] = seg[y + 1, x] = a
                    else:
                        seg[y, x] = seg[y + 1, x + 1] = a
                    out.append(seg)
    return out


def strips(kmax=12):
    """1 x n strips of distinct ids for n = 2^k - 2, 2^k - 1, 2^k, k = 1 .. kmax, on every other row: rings of
    2 n + 2 edges.  (lengths, raster)"""
    lengths = [n for k in range(1, kmax + 1) for n in (2 ** k - 2, 2 ** k - 1, 2 ** k) if n > 0]
    seg = np.zeros((2 * len(lengths), max(lengths) + 3), dtype=np.uint32)
    for (i, n) in enumerate(lengths):
        x0 = i % 3
        seg[2 * i, x0:x0 + n] = i + 1
    return (lengths, seg)


def serpentine(n=512):
    """a one-pixel corridor of id 1 winding between walls of id 2: one ring of more than n^2 / 2 edges whose leader
    lies at column n - 1 of the first row"""
    seg = np.full((n, n), 2, dtype=np.uint32)
    seg[1::2, :] = 1
    seg[0, :] = 2
    seg[0, n - 1] = 1
    for (j, y) in enumerate(range(2, n, 2)):
        seg[y, 0 if j % 2 == 0 else n - 1] = 1
    return seg


def staircase(n=70):
    (y, x) = np.indices((n, n))
    return np.where(x <= y, 1, 2).astype(np.uint32)


def long_strips(n=4096):
    return (np.ones((1, n), dtype=np.uint32), np.ones((n, 1), dtype=np.uint32))


def concentric_squares(ids=(1, 2, 1, 2, 1), width=2):
    n = 2 * width * len(ids) - width
    seg = np.zeros((n, n), dtype=np.uint32)
    for (k, i) in enumerate(ids):
        seg[k * width:n - k * width, k * width:n - k * width] = i
    return seg


def scattered_parts(parts=300, seed=11):
    """id 7 in `parts` single pixels scattered among the ids 1 .. 6 and 8 .. 20"""
    rng = np.random.default_rng(seed)
    others = np.array([1, 2, 3, 4, 5, 6, 8, 9, 10, 15, 20], dtype=np.uint32)
    seg = others[rng.integers(0, len(others), size=(90, 150))]
    (ys, xs) = np.meshgrid(np.arange(1, 90, 3), np.arange(1, 150, 3), indexing='ij')
    pick = rng.permutation(ys.size)[:parts]
    seg[ys.ravel()[pick], xs.ravel()[pick]] = 7
    return seg


def last_pixel_only():
    seg = np.ones((37, 70), dtype=np.uint32)
    seg[-1, -1] = 5
    return seg
