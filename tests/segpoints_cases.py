"""The cases of tests/test_gpu_segpoints_edges.py and tests/test_gpu_dsegpoints_edges.py -- the per-segment point lists
of csrc/segpoints.h and csrc/dsegpoints.h at their run, tile, value and shard edges -- with two models in plain numpy.

Importable without a GPU: tests/test_segpoints_cases_host.py asserts, from run_model, that every builder reaches the
edge it was built for, so a later edit to a builder cannot lose its edge unnoticed.  The expected point lists always
come from visit_points (segpoints_helpers.visit_points on a whole raster, the slice form below on a shard); run_model
is never compared with device output: the run table is not visible outside the library.

Every builder returns ((seg, band, null, S, tile), props): label raster (uint32), band, nodata value, maxSegId, tile
size, and the properties it was built for.  Everything is integer work: numpy.array_equal with dtype, no tolerance.
"""
import os
import re

import numpy as np

import segpoints_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'pyshepseg_amd', 'csrc')

DTYPES = (np.uint8, np.int16, np.uint16, np.int32, np.uint32)
WAVE = 64               # a run is cut at every multiple of 64 visit indices; one wavefront expands 64 sorted runs
EXPAND_BLOCK = 256      # sorted runs per workgroup of k_pts_expand / k_dpts_expand
SCAN_BLOCK = 8192       # items of one block of scan.h's prefix sum (tests/prim_cases.py derives it from the header)
MAX_PIXELS = 66000      # no raster of the one-GPU file is larger


def constants():
    """(PTS_TILE, PTS_ROWS) as csrc/segpoints.h defines them"""
    text = open(os.path.join(CSRC, 'segpoints.h')).read()
    out = []
    for name in ('PTS_TILE', 'PTS_ROWS'):
        m = re.search(r'^#define\s+%s\s+(\d+)u?\b' % name, text, flags=re.M)
        assert m, 'no #define %s' % name
        out.append(int(m.group(1)))
    return tuple(out)


# ---- the two models -----------------------------------------------------------------------------------------------
def visit_key(rows, cols, img_rows, ncols, tile):
    """The global visit index (int64) of pixels (rows, cols) of an img_rows x ncols raster that need not exist, by the
    definition in segpoints.h: bands of `tile` image rows one after the other, in a band its tiles (all `tile` wide but
    the last), in a tile its rows.  Every earlier band is full, and so is every earlier tile of a band."""
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    th = max(1, min(int(tile), int(img_rows)))
    tw = max(1, min(int(tile), int(ncols)))
    y0 = rows - rows % th
    hb = np.minimum(th, img_rows - y0)
    x0 = cols - cols % tw
    w = np.minimum(tw, ncols - x0)
    return y0 * ncols + x0 * hb + (rows - y0) * w + (cols - x0)


def visit_points(seg, band, null_val, tile, max_seg_id=None, row0=0, img_rows=None, with_key=False):
    """segpoints_helpers.visit_points for a slice: seg / band are rows [row0, row0 + len(seg)) of an img_rows-row
    raster, the points come stably sorted by id in the WHOLE raster's visit order (visit_key), y is the row of the
    whole raster.  On a whole raster (the defaults) it equals segpoints_helpers.visit_points.  with_key: the points'
    visit indices as a fifth array."""
    seg = np.asarray(seg)
    (nr, nc) = seg.shape
    if img_rows is None:
        img_rows = row0 + nr
    if max_seg_id is None:
        max_seg_id = int(seg.max()) if seg.size else 0
    (r, c) = np.indices((nr, nc), dtype=np.int64)
    r += row0
    key = visit_key(r, c, img_rows, nc, tile)
    valid = (seg != 0) & (seg <= max_seg_id)
    if null_val is not None:
        valid &= band.astype(np.int64) != int(null_val)
    ids = seg[valid].astype(np.int64)
    order = np.lexsort((key[valid], ids))
    out = (ids[order], c[valid][order], r[valid][order], band[valid].astype(np.int64)[order])
    return out + (key[valid][order],) if with_key else out


def slice_geom(row0, nrows, img_rows, tile):
    """(th, h0) of pts_geom_slice: the band height, and the rows of the slice's first band"""
    th = min(int(tile), int(img_rows))
    left = th - row0 % th if th else 0
    return th, min(left, nrows)


def run_model(seg, band, null, tile, S, row0=0, img_rows=None):
    """The runs as k_pts_run_emit cuts them.  The slice's pixels in ascending global visit index are its local visit
    indices 0 .. n - 1; a pixel is a point when its label is in 1..S and its value is not `null`; a run is a maximal
    stretch of consecutive local visit indices with one point id, cut at every multiple of 64 and at every tile-row
    start.  Returns a dict: n, m, npts, heads (local visit index of every run's first pixel), lanes (heads % 64),
    lens, ids, pos (raster position of the head), all in visit order; order (the stable order by id), sids / slens
    (ids and lens in that order), key (the n pixels' point ids in visit order, 0 where there is no point)."""
    seg = np.asarray(seg)
    (nr, nc) = seg.shape
    n = nr * nc
    if img_rows is None:
        img_rows = row0 + nr
    (r, c) = np.indices((nr, nc), dtype=np.int64)
    gkey = visit_key(r + row0, c, img_rows, nc, tile).ravel()
    pos = np.argsort(gkey, kind='stable')                   # local visit index -> raster position
    assert n == 0 or (np.diff(gkey[pos]) > 0).all()
    tw = max(1, min(int(tile), nc))
    ids = seg.ravel()[pos].astype(np.int64)
    point = (ids != 0) & (ids <= S)
    if null is not None:
        point &= np.asarray(band).ravel()[pos].astype(np.int64) != int(null)
    key = np.where(point, ids, 0)
    i = np.arange(n, dtype=np.int64)
    row_start = (pos % max(nc, 1)) % tw == 0
    bound = (i % WAVE == 0) | (key != np.r_[np.zeros(1, np.int64), key[:-1]]) | row_start
    heads = np.flatnonzero(bound & (key != 0))
    nxt = np.r_[np.flatnonzero(bound), n]                    # (the raster's end ends a run too)
    end = nxt[np.searchsorted(nxt, heads, side='right')]
    end = np.minimum(end, np.minimum((heads // WAVE + 1) * WAVE, n))
    lens = end - heads
    assert (pos[end - 1] == pos[heads] + lens - 1).all()     # a run is consecutive pixels of one image row
    assert int(lens.sum()) == int(point.sum())
    order = np.argsort(key[heads], kind='stable')
    return {'n': n, 'm': len(heads), 'npts': int(lens.sum()), 'heads': heads, 'lanes': heads % WAVE, 'lens': lens,
            'ids': key[heads], 'pos': pos[heads], 'order': order, 'sids': key[heads][order], 'slens': lens[order],
            'key': key}


def run_ranges(model, S):
    """first sorted run of every id 0 .. S + 1 (the rlo / rhi k_pts_range finds for an id range)"""
    return np.searchsorted(model['sids'], np.arange(S + 2))


# ---- the geometry sweep -------------------------------------------------------------------------------------------
SHAPES = ((1, 1), (1, 200), (200, 1), (5, 64), (5, 65), (3, 127), (3, 128), (3, 129), (63, 65), (64, 64), (17, 241),
          (65, 129))
TILES = (1, 2, 63, 64, 65, 128, 10 ** 6)


def _geometry_pairs():
    """Every (shape, tile) whose tile, cut to the raster as pts_geom cuts it (th = min(tile, rows), tw = min(tile,
    cols)), differs from that of a smaller tile of the list: the kernels see th and tw only, so a dropped pair is the
    same launch as the pair kept.  Dropped are, per shape, the larger tiles that cover the raster as the first one
    does -- (1, 1) beyond tile 1; (5, 64) and (64, 64) beyond 64; (1, 200) and (200, 1) at 10^6 (as 128 on the short
    side, but 128 < 200 on the long one: kept are 1 .. 128 and 10^6 there); (5, 65), (63, 65) beyond 65; (3, 127),
    (3, 128) beyond 128; (3, 129), (17, 241), (65, 129) keep all seven."""
    kept, dropped = [], []
    for (rows, cols) in SHAPES:
        seen = set()
        for tile in TILES:
            cut = (min(tile, rows), min(tile, cols))
            (dropped if cut in seen else kept).append((rows, cols, tile))
            seen.add(cut)
    return kept, dropped


GEOMETRY, GEOMETRY_DROPPED = _geometry_pairs()
PER_PIXEL = (65, 129, 64)           # the pair that also runs with one id per pixel: 8385 runs of one pixel


def field(rows, cols, seed, dtype=np.uint8, null=0, nids=9, block=(3, 5)):
    """ids 1..nids in small random blocks, a tenth of the pixels unlabelled, a tenth nodata"""
    rng = np.random.RandomState(seed)
    base = rng.randint(1, nids + 1, size=(rows // block[0] + 1, cols // block[1] + 1))
    seg = np.kron(base, np.ones(block, dtype=np.int64))[:rows, :cols].astype(np.uint32)
    seg[rng.rand(rows, cols) < 0.1] = 0
    band = rng.randint(1, 200, size=(rows, cols)).astype(dtype)
    band[rng.rand(rows, cols) < 0.1] = null
    return np.ascontiguousarray(seg), np.ascontiguousarray(band)


def geometry(rows, cols, tile, per_pixel=False):
    if per_pixel:
        seg = np.arange(1, rows * cols + 1, dtype=np.uint32).reshape(rows, cols)
        band = ((np.arange(rows * cols) * 7) % 251 + 1).astype(np.uint8).reshape(rows, cols)
        S = rows * cols
    else:
        (seg, band) = field(rows, cols, rows * 1000 + cols)
        S = 9
    (th, tw) = (min(tile, rows), min(tile, cols))
    props = {'n': rows * cols, 'last_col_width': cols - (cols - 1) // tw * tw,
             'last_band_rows': rows - (rows - 1) // th * th}
    return (seg, band, 0, S, tile), props


# ---- ballot edges -------------------------------------------------------------------------------------------------
def ballot_plain():
    """one id on 6 x 200, tile 200: one tile, visit index == raster index, row starts at 200, 400, ... off the
    64 grid; n = 1200 is no multiple of 64 and the last pixels are points"""
    seg = np.ones((6, 200), dtype=np.uint32)
    band = np.full((6, 200), 7, dtype=np.uint8)
    return (seg, band, 0, 1, 200), {'n': 1200, 'tail': 1200 % WAVE}


def ballot_marks():
    """ballot_plain with: a pixel of id 2 at every visit index 63 mod 64 of the first three 64-groups and at 1151;
    a zero at visit index 128 and 640 (0 mod 64); 64-group 4 all zero, group 5 all nodata, group 7 all zero but its
    last lane"""
    ((seg, band, null, _S, tile), _p) = ballot_plain()
    s = seg.reshape(-1)
    b = band.reshape(-1)
    for i in (63, 127, 191, 1151):
        s[i] = 2
    s[128] = 0
    s[640] = 0
    s[4 * 64:5 * 64] = 0
    b[5 * 64:6 * 64] = null
    s[7 * 64:8 * 64 - 1] = 0
    return (seg, band, null, 2, tile), {'n': 1200, 'tail': 1200 % WAVE, 'empty_groups': (4, 5)}


def ballot_all_64():
    """one id on 64 x 64, tile 64: every run is exactly 64 from lane 0"""
    seg = np.ones((64, 64), dtype=np.uint32)
    band = (np.arange(4096) % 250 + 1).astype(np.uint8).reshape(64, 64)
    return (seg, band, 0, 1, 64), {'n': 4096, 'm': 64}


# ---- expansion ----------------------------------------------------------------------------------------------------
def expand_one_id(side):
    """side x side of one id, tile 64: side * side / 64 runs of 64 (side 64: one wavefront's 4096 records; side 128:
    256 runs, a full workgroup)"""
    seg = np.ones((side, side), dtype=np.uint32)
    band = ((np.arange(side * side) * 3) % 65521 + 1).astype(np.uint16).reshape(side, side)
    return (seg, band, 0, 1, 64), {'m': side * side // 64, 'npts': side * side}


def pack_runs(specs, cols=256):
    """Labels whose runs are exactly `specs` ((id, length <= 64) in visit order) on a raster `cols` wide (a multiple
    of 64) visited as one tile: a run never crosses a multiple of 64, a zero follows every run that does not end on
    one."""
    assert cols % WAVE == 0
    out = []
    for (i, length) in specs:
        at = len(out) % WAVE
        if at + length > WAVE:
            out += [0] * (WAVE - at)
        out += [i] * length
        if len(out) % WAVE:
            out.append(0)
    rows = max(1, -(-len(out) // cols))
    seg = np.zeros(rows * cols, dtype=np.uint32)
    seg[:len(out)] = out
    return seg.reshape(rows, cols)


EXPAND_RUNS = {1: 5, 2: 63, 3: 64, 4: 65, 5: 255, 6: 256, 7: 257}         # sorted runs per id


def _expand_len(i, j):
    return {1: 1, 2: 1, 3: 64, 4: 1, 5: 1 if j % 2 else 64, 6: 33, 7: (j * 7) % 64 + 1}[i]


def expand_mixed():
    """Seven ids whose sorted-run counts are 5, 63, 64, 65, 255, 256 and 257, so that an emit of one id has rhi - rlo
    of each and an rlo (5, 68, 132, 197, 452, 708) that is no multiple of 256; id 3 is 64 runs of 64 (4096 records
    from 64 consecutive sorted runs), ids 5 and 7 mix lengths 1 .. 64 inside a wavefront.  The runs of the ids
    interleave in visit order, so the sort moves every one of them."""
    specs = []
    for j in range(max(EXPAND_RUNS.values())):
        for i in (3, 5, 6, 7, 1, 2, 4):
            if j < EXPAND_RUNS[i]:
                specs.append((i, _expand_len(i, j)))
    seg = pack_runs(specs)
    band = ((np.arange(seg.size) * 11) % 65521 + 1).astype(np.uint16).reshape(seg.shape)
    return (seg, band, 0, 7, 10 ** 6), {'runs': dict(EXPAND_RUNS)}


def expand_between():
    """long runs of id 2 (64 each) that sort between single pixels of id 1 and of id 3"""
    specs = []
    for j in range(96):
        specs += [(1, 1), (3, 1)] * 3 + [(2, 64)]
    seg = pack_runs(specs, cols=128)
    band = ((np.arange(seg.size) * 5) % 250 + 1).astype(np.uint8).reshape(seg.shape)
    return (seg, band, 0, 3, 128), {'runs': {1: 288, 2: 96, 3: 288}}


# ---- ids ----------------------------------------------------------------------------------------------------------
def ids_above_max():
    """labels 1..9 with maxSegId 5: the pixels of 6..9 are ignored (and cut the runs of the others)"""
    (seg, band) = field(20, 70, 11)
    return (seg, band, 0, 5, 16), {'ignored': (6, 7, 8, 9)}


def ids_single():
    (seg, band) = field(9, 70, 12, nids=1)
    return (seg, band, 0, 1, 8), {}


def ids_sparse_large():
    """S = 2^20 with five ids present: the first, the last, and three in between"""
    S = 1 << 20
    present = np.array([1, 255, 256, 70000, S], dtype=np.uint32)
    rng = np.random.RandomState(5)
    seg = present[rng.randint(0, 5, size=(12, 70))]
    seg[rng.rand(12, 70) < 0.1] = 0
    band = rng.randint(0, 200, size=(12, 70)).astype(np.uint8)
    return (np.ascontiguousarray(seg), band, 0, S, 16), {'present': present}


def ids_gaps():
    """ids without pixels first (1, 2), in between (5, 6, 8, 9) and last (11, 12); id 7 has pixels that are all
    nodata"""
    rng = np.random.RandomState(6)
    present = np.array([3, 4, 7, 10], dtype=np.uint32)
    seg = np.ascontiguousarray(present[rng.randint(0, 4, size=(10, 66))])
    band = rng.randint(1, 200, size=(10, 66)).astype(np.int16)
    band[seg == 7] = -3
    return (seg, band, -3, 12, 4), {'present': (3, 4, 10), 'pointless': (7,)}


def empty(kind):
    """rasters without a point: all labels zero, all values nodata, no rows, no columns"""
    shape = {'zero': (7, 70), 'nodata': (7, 70), 'norows': (0, 70), 'nocols': (7, 0)}[kind]
    seg = np.zeros(shape, dtype=np.uint32) if kind == 'zero' else np.full(shape, 2, dtype=np.uint32)
    band = np.full(shape, 9, dtype=np.uint16)
    return (seg, band, 9 if kind != 'zero' else 0, 3, 8), {'n': shape[0] * shape[1]}


# ---- values -------------------------------------------------------------------------------------------------------
def edge_values(dtype):
    """the type's minimum, maximum, 0 and the values next to them; the sign bit of every narrower width"""
    info = np.iinfo(dtype)
    cand = [info.min, info.min + 1, info.min + 2, -2, -1, 0, 1, 2, info.max - 2, info.max - 1, info.max,
            127, 128, 255, 256, 32767, 32768, 65535, 65536, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, -2 ** 31, -32768, -32769]
    return sorted({v for v in cand if info.min <= v <= info.max})


def value_nulls(dtype):
    """nodata at each limit in turn, then outside the pixel type's range (nothing is nodata then)"""
    info = np.iinfo(dtype)
    outside = [info.max + 1, info.min - 1]
    if info.min == 0:
        outside.append(-1)
    if info.bits == 16:
        outside.append(70000)
    if dtype == np.uint32:
        outside.append(2 ** 32)
    return [info.min, info.max] + sorted(set(outside))


def values(dtype, null, stripes=False):
    """5 x 67 of the type's edge values, ids 1..4 in blocks with some zeros, tile 64 (a last tile column 3 wide);
    stripes: ids 1..6 as vertical stripes over all rows (every id on every row shard)"""
    vals = np.array(edge_values(dtype), dtype=np.int64)
    band = np.resize(vals, (5, 67)).astype(dtype)
    cols = np.arange(67)
    if stripes:
        seg = np.broadcast_to((cols // 3 % 6 + 1).astype(np.uint32), (5, 67)).copy()
        S = 6
    else:
        seg = ((cols[None, :] // 7 + np.arange(5)[:, None] // 2) % 4 + 1).astype(np.uint32)
        seg[:, 13::17] = 0
        S = 4
    return (seg, band, null, S, 64), {'values': vals}


# ---- row shards (tests/test_gpu_dsegpoints_edges.py) --------------------------------------------------------------
SLICE_ROWS = 40
# the cuts of a 40-row raster against bands of 8 rows: row ranges per rank ((0, 0): a rank without rows)
SLICE_CUTS = {
    'band-edge': [(0, 16), (16, 40)],
    'row-after': [(0, 17), (17, 40)],
    'row-before': [(0, 15), (15, 40)],
    'inside-one-band': [(0, 18), (18, 21), (21, 40)],
    'one-row': [(0, 24), (24, 25), (25, 40)],
    'empty-first': [(0, 0), (0, 19), (19, 40)],
    'empty-middle': [(0, 19), (0, 0), (19, 40)],
    'empty-last': [(0, 19), (19, 40), (0, 0)],
}
SLICE_TILES = (8, 1, 64, 16)      # 1: every row a band; 64: one band; 16: the last band is half a band (8 rows)


def slice_raster(cols=70):
    """40 rows of small blocks (segments complete on a rank, whatever the cut) between vertical streaks (on every
    rank); 70 columns: the last tile column of tile 8 is 6 wide, of tile 64 too.  129 columns with tile 128: one wide."""
    rng = np.random.RandomState(40 + cols)
    base = rng.randint(1, 30, size=(SLICE_ROWS // 4 + 1, cols // 5 + 1))
    seg = np.kron(base, np.ones((4, 5), dtype=np.int64))[:SLICE_ROWS, :cols]
    seg = seg + (np.arange(SLICE_ROWS)[:, None] // 4) * 30       # a block id never comes back in a later row of blocks
    streak = np.arange(cols) % 11 == 3
    seg[:, streak] = 400 + np.arange(cols)[streak][None, :] // 11
    seg = seg.astype(np.uint32)
    seg[rng.rand(SLICE_ROWS, cols) < 0.03] = 0
    band = rng.randint(1, 3000, size=(SLICE_ROWS, cols)).astype(np.uint16)
    band[rng.rand(SLICE_ROWS, cols) < 0.1] = 0
    return (np.ascontiguousarray(seg), band, 0, int(seg.max()) + 2, None), {}


def _band16(shape):
    return ((np.arange(shape[0] * shape[1]) * 13) % 65521 + 1).astype(np.uint16).reshape(shape)


def records_one_id():
    """one id over 40 x 300: with any cut its 12 000 points all travel, in runs of 64 (tile 64)"""
    seg = np.ones((40, 300), dtype=np.uint32)
    return (seg, _band16(seg.shape), 0, 1, 64), {'records': 12000}


def records_stripes():
    """vertical stripes 3 wide: every id is on every rank"""
    seg = np.broadcast_to((np.arange(300) // 3 + 1).astype(np.uint32), (40, 300)).copy()
    return (seg, _band16(seg.shape), 0, 100, 16), {}


def records_bands():
    """horizontal bands of 10 rows cut on their edges: no id on two ranks, no record, slot 0"""
    seg = np.broadcast_to((np.arange(40) // 10 + 1).astype(np.uint32)[:, None], (40, 300)).copy()
    return (seg, _band16(seg.shape), 0, 4, 16), {'cuts': [(0, 20), (20, 40)]}


def records_alternating():
    """columns in stripes 2 wide, cut at row 20: odd ids run down all 40 rows (straddlers), even ids 2k hold the
    stripe's upper half and 2k + 150 its lower half (complete on one rank).  A rank's sorted runs then alternate
    straddler and complete every 20 runs: inside each wavefront of k_dpts_expand the zero-length runs of the
    straddlers share a prefix with the complete run after them."""
    cols = np.arange(300)
    stripe = cols // 2 + 1                                  # 1 .. 150
    seg = np.broadcast_to(stripe.astype(np.uint32), (40, 300)).copy()
    even = stripe % 2 == 0
    seg[20:, even] += 150
    return (seg, _band16(seg.shape), 0, 300, 1024), {'cuts': [(0, 20), (20, 40)]}


def id_range(rank, world, S):
    """distdev.idRange, restated (host tests need it without the package)"""
    ns = int(S) + 1
    return (rank * ns) // world, ((rank + 1) * ns) // world


SHARE_CASES = ((3, 9), (4, 3), (4, 2), (3, 12))         # (world, S)


def shares(world, S):
    """Every share's first and last id (id_lo, id_hi - 1; id 0 is nobody's segment) is a vertical stripe over all 40
    rows -- a straddler under any cut -- and every other id a block of the first ten rows, complete on rank 0.
    (3, 9): shares of 3, 3 and 4 ids; (4, 3): every share exactly one id, rank 0's the id 0, which holds no segment;
    (4, 2): rank 0's share is empty, (0, 0); (3, 12): 4, 4 and 5 ids."""
    strad = set()
    for r in range(world):
        (lo, hi) = id_range(r, world, S)
        if hi > lo:
            strad |= {lo, hi - 1}
    strad.discard(0)
    seg = np.zeros((40, 6 * S + 2), dtype=np.uint32)
    for i in range(1, S + 1):
        if i in strad:
            seg[:, 6 * (i - 1) + 1:6 * (i - 1) + 4] = i
        else:
            seg[2:9, 6 * (i - 1) + 1:6 * (i - 1) + 5] = i
    sizes = [hi - lo for (lo, hi) in (id_range(r, world, S) for r in range(world))]
    cuts = [(r * 40 // world, (r + 1) * 40 // world) for r in range(world)]
    return (seg, _band16(seg.shape), 0, S, 4), {'straddlers': sorted(strad), 'share_sizes': sizes, 'cuts': cuts}


# ---- visit indices of 2^32 and above ------------------------------------------------------------------------------
BIG = {'img_rows': 65536, 'ncols': 65537, 'tile': 8, 'rows': ((65528, 65532), (65532, 65536)), 'S': 3,
       'band_start': 4294508536, 'x0': 57344}


def big_visit_shards():
    """The two 4-row shards of the last band of a 65536 x 65537 raster that is never materialised.  id 1: columns
    57336..57351 of all eight rows (two tile columns; the second one's indices cross 2^32 at its ninth pixel, so the
    straddler's records interleave across both ranks and across 2^32); id 2: complete on rank 0; id 3: complete on
    rank 1, reaching into the last tile column, one pixel wide.  Returns [(seg, band, row0)] and the global
    histogram."""
    nc = BIG['ncols']
    out = []
    hist = np.zeros(BIG['S'] + 1, dtype=np.uint32)
    for (r, (lo, hi)) in enumerate(BIG['rows']):
        seg = np.zeros((hi - lo, nc), dtype=np.uint32)
        seg[:, 57336:57352] = 1
        if r == 0:
            seg[1:4, 100:121] = 2
        else:
            seg[0:3, nc - 9:nc] = 3
        (y, x) = np.indices(seg.shape)
        band = ((x * 3 + (y + lo) * 5) % 65521 + 1).astype(np.uint16)
        band[:, 57340] = 0                                   # nodata inside the straddler
        hist += np.bincount(seg.ravel(), minlength=BIG['S'] + 1).astype(np.uint32)
        out.append((seg, band, lo))
    hist[0] = 0
    return out, hist
