"""Host: the builders of tests/segpoints_cases.py reach the edges they claim (asserted from run_model), visit_key
orders as segpoints_helpers.visit_points does, and the arithmetic of the 2^32 case holds.  No GPU: this file must pass
before tests/test_gpu_segpoints_edges.py and tests/test_gpu_dsegpoints_edges.py are trusted."""
import numpy as np
import pytest

import segpoints_cases as C
import segpoints_helpers as H


def _same_points(a, b):
    return len(a) == len(b) and all(np.array_equal(p, q) and p.dtype == q.dtype for (p, q) in zip(a, b))


def test_constants_are_what_the_builders_assume():
    assert C.constants() == (4096, 16)
    assert C.constants()[0] == 4 * C.constants()[1] * C.WAVE
    from prim_cases import SCAN_ITEMS
    assert C.SCAN_BLOCK == SCAN_ITEMS == 8192


# ---- visit_key against visit_points ------------------------------------------------------------------------------
def _slices_agree(seg, band, null, tile, S):
    rows = seg.shape[0]
    whole = C.visit_points(seg, band, null, tile, S)
    assert _same_points(whole, H.visit_points(seg, band, null, tile, S))
    for a in range(rows):
        for b in sorted({a + 1, min(a + min(tile, rows) + 1, rows), rows}):
            got = C.visit_points(seg[a:b], band[a:b], null, tile, S, row0=a, img_rows=rows)
            keep = (whole[2] >= a) & (whole[2] < b)
            assert _same_points(got, tuple(w[keep] for w in whole)), (a, b)


@pytest.mark.parametrize('seed', range(12))
def test_visit_key_orders_as_visit_points_random(seed):
    rng = np.random.RandomState(seed)
    (rows, cols, tile) = (rng.randint(1, 30), rng.randint(1, 40), rng.randint(1, 20))
    (seg, band) = C.field(rows, cols, seed, block=(2, 3))
    _slices_agree(seg, band, 0, tile, 9)
    # the key is the rank of the pixel among all pixels in the padded-tile order of visit_points
    (r, c) = np.indices((rows, cols), dtype=np.int64)
    ntc = -(-cols // tile)
    padded = (((r // tile) * ntc + c // tile) * tile + r % tile) * tile + c % tile
    key = C.visit_key(r, c, rows, cols, tile)
    assert np.array_equal(np.argsort(padded.ravel()), np.argsort(key.ravel()))
    assert np.array_equal(np.sort(key.ravel()), np.arange(rows * cols))


@pytest.mark.parametrize('rows,cols,tile', C.GEOMETRY)
def test_visit_key_orders_as_visit_points_sweep(rows, cols, tile):
    ((seg, band, null, S, _t), _p) = C.geometry(rows, cols, tile)
    _slices_agree(seg, band, null, tile, S)


def _visit_pos(i, nrows, ncols, th, tw, h0):
    """pts_visit_pos of segpoints.h, line by line: (raster position, row start)"""
    first = h0 * ncols
    if i < first:
        (rem, y0, h) = (i, 0, h0)
    else:
        bandsz = th * ncols
        tr = (i - first) // bandsz
        rem = i - first - tr * bandsz
        y0 = h0 + tr * th
        h = min(th, nrows - y0)
    tilesz = h * tw
    tc = rem // tilesz
    rem -= tc * tilesz
    x0 = tc * tw
    w = min(tw, ncols - x0)
    (rr, cc) = divmod(rem, w)
    return (y0 + rr) * ncols + x0 + cc, cc == 0


@pytest.mark.parametrize('rows,cols,tile', [g for g in C.GEOMETRY if g[0] * g[1] <= 1300])
def test_device_visit_position_equals_the_key_order(rows, cols, tile):
    """the kernel's index arithmetic, transcribed, visits every slice in ascending visit_key"""
    tw = min(tile, cols)
    for a in range(rows):
        for b in sorted({a + 1, min(a + 2, rows), min(a + min(tile, rows), rows), rows}):
            (th, h0) = C.slice_geom(a, b - a, rows, tile)
            n = (b - a) * cols
            got = [_visit_pos(i, b - a, cols, th, tw, h0) for i in range(n)]
            (r, c) = np.indices((b - a, cols), dtype=np.int64)
            want = np.argsort(C.visit_key(r + a, c, rows, cols, tile).ravel(), kind='stable')
            assert np.array_equal([g[0] for g in got], want), (a, b)
            assert np.array_equal([g[1] for g in got], (want % cols) % tw == 0), (a, b)


# ---- the geometry sweep ------------------------------------------------------------------------------------------
def test_sweep_holds_every_shape_and_the_stated_edges():
    assert len(C.GEOMETRY) + len(C.GEOMETRY_DROPPED) == len(C.SHAPES) * len(C.TILES)
    assert {(r, c) for (r, c, _t) in C.GEOMETRY} == set(C.SHAPES)
    for (rows, cols, tile) in C.GEOMETRY_DROPPED:           # a dropped pair is the launch of a kept one
        assert any((r, c) == (rows, cols) and t < tile and min(t, rows) == min(tile, rows) and
                   min(t, cols) == min(tile, cols) for (r, c, t) in C.GEOMETRY)
    for tile in C.TILES:                                     # every tile size meets a raster larger than it, or all of them
        assert any(t == tile for (_r, _c, t) in C.GEOMETRY)
    props = [C.geometry(*g)[1] for g in C.GEOMETRY]
    ns = {p['n'] for p in props}
    assert {4095, 4096, 4097} <= ns and min(ns) == 1
    assert any(C.SCAN_BLOCK // 2 < n < C.SCAN_BLOCK for n in ns) and any(n > C.SCAN_BLOCK for n in ns)
    assert max(ns) <= C.MAX_PIXELS
    assert any(p['last_col_width'] == 1 and g[1] > 1 and g[2] > 1 for (g, p) in zip(C.GEOMETRY, props))
    assert any(p['last_band_rows'] == 1 and g[0] > 1 and g[2] > 1 for (g, p) in zip(C.GEOMETRY, props))
    assert any(p['last_col_width'] == 1 and p['last_band_rows'] == 1 and g[2] == 64 for (g, p) in zip(C.GEOMETRY, props))
    for want in ((1, 1, 1), (1, 200, 1), (200, 1, 1), (200, 1, 10 ** 6), (1, 200, 10 ** 6), (64, 64, 64), (64, 64, 63),
                 (5, 65, 64), (5, 65, 65), (3, 129, 128), (17, 241, 10 ** 6), (65, 129, 64)):
        assert want in C.GEOMETRY, want


def test_sweep_rasters_have_points_holes_and_runs_cut_by_tile_rows():
    for g in C.GEOMETRY:
        ((seg, band, null, S, tile), p) = C.geometry(*g)
        m = C.run_model(seg, band, null, tile, S)
        assert m['n'] == p['n'] == g[0] * g[1]
        if p['n'] >= 64:
            assert 0 < m['npts'] < m['n'] and (seg == 0).any() and (band == null).any()
    ((seg, band, null, S, tile), p) = C.geometry(*C.PER_PIXEL, per_pixel=True)
    m = C.run_model(seg, band, null, tile, S)
    assert m['m'] == m['npts'] == m['n'] == 8385 > C.SCAN_BLOCK and (m['lens'] == 1).all() and S == 8385
    assert C.PER_PIXEL in C.GEOMETRY


# ---- ballot edges ------------------------------------------------------------------------------------------------
def test_ballot_plain_rows_start_off_the_grid_and_the_tail_is_valid():
    ((seg, band, null, S, tile), p) = C.ballot_plain()
    m = C.run_model(seg, band, null, tile, S)
    assert m['n'] == 1200 and m['n'] % 64 == 48 == p['tail'] and m['npts'] == 1200
    starts = set(range(200, 1200, 200))
    assert all(s % 64 for s in starts) and starts <= set(m['heads'].tolist())
    assert set(m['heads'].tolist()) == starts | set(range(0, 1200, 64))
    # the final run ends at the raster's end inside a wavefront
    assert m['heads'][-1] == 1152 and m['lens'][-1] == 48 and m['key'][-1] == 1
    # runs of exactly 64 from lane 0, and runs that a row start cuts on either side
    assert ((m['lanes'] == 0) & (m['lens'] == 64)).sum() >= 10
    assert ((m['lanes'] == 0) & (m['lens'] < 64)).any() and ((m['lanes'] > 0) & (m['lanes'] + m['lens'] == 64)).any()


def test_ballot_marks_reach_lane_63_zero_on_lane_0_and_empty_rows():
    ((seg, band, null, S, tile), p) = C.ballot_marks()
    m = C.run_model(seg, band, null, tile, S)
    heads = dict(zip(m['heads'].tolist(), zip(m['ids'].tolist(), m['lens'].tolist())))
    for i in (63, 127, 191, 1151):
        assert i % 64 == 63 and heads[i] == (2, 1)                 # another id's head on lane 63
    assert heads[511] == (1, 1)                                    # the only point of its row of 64, on lane 63
    for i in (128, 640):
        assert m['key'][i] == 0 and i not in heads and heads[i + 1][0] == 1        # a zero at 0 mod 64
    for g in p['empty_groups']:                                    # rows of 64 without a head: all zero, all nodata
        assert not any(g * 64 <= h < (g + 1) * 64 for h in heads)
    assert (seg.reshape(-1)[4 * 64:5 * 64] == 0).all() and (seg.reshape(-1)[5 * 64:6 * 64] == 1).all()
    assert (band.reshape(-1)[5 * 64:6 * 64] == null).all()
    assert heads[64] == (1, 63) and heads[0] == (1, 63)            # a run that lane 63's other id ends
    assert m['n'] % 64 == 48 and m['key'][-1] == 1 and m['heads'][-1] == 1152 and m['lens'][-1] == 48
    assert heads[1088] == (1, 63) and heads[1000][1] == 24         # row start at 1000, the grid at 1024


def test_ballot_all_64_is_the_rest_zero_path():
    ((seg, band, null, S, tile), p) = C.ballot_all_64()
    m = C.run_model(seg, band, null, tile, S)
    assert m['m'] == 64 == p['m'] and (m['lens'] == 64).all() and (m['lanes'] == 0).all() and m['n'] == 4096


# ---- expansion ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('side,runs', [(64, 64), (128, 256)])
def test_expand_one_id_fills_a_wavefront_then_a_workgroup(side, runs):
    ((seg, band, null, S, tile), p) = C.expand_one_id(side)
    m = C.run_model(seg, band, null, tile, S)
    assert m['m'] == runs == p['m'] and (m['lens'] == 64).all() and m['npts'] == runs * 64
    assert m['slens'][:64].sum() == 4096 == C.constants()[0]        # 64 consecutive sorted runs holding 4096 points
    assert runs in (C.WAVE, C.EXPAND_BLOCK)


def test_expand_mixed_run_counts_and_starts():
    ((seg, band, null, S, tile), p) = C.expand_mixed()
    assert seg.size <= C.MAX_PIXELS and seg.shape[1] % 64 == 0
    m = C.run_model(seg, band, null, tile, S)
    starts = C.run_ranges(m, S)
    counts = np.diff(starts)[1:S + 1]
    assert counts.tolist() == [5, 63, 64, 65, 255, 256, 257] == [p['runs'][i] for i in range(1, 8)]
    assert starts[2:S + 1].tolist() == [5, 68, 132, 197, 452, 708]
    assert all(int(s) % C.EXPAND_BLOCK for s in starts[2:S + 1])    # rlo of ids 2 .. 7 is no multiple of 256
    assert m['m'] == 965 and m['npts'] > 3 * C.SCAN_BLOCK
    # id 3: 64 consecutive sorted runs holding 4096 points; ids 5 and 7 mix lengths inside a wavefront
    assert (m['slens'][starts[3]:starts[4]] == 64).all() and m['slens'][starts[3]:starts[4]].sum() == 4096
    assert set(m['slens'][starts[5]:starts[6]].tolist()) == {1, 64}
    assert len(set(m['slens'][starts[7]:starts[7] + 64].tolist())) == 64
    # the runs interleave in visit order: the sort moves them
    assert (np.diff(m['ids'][:50]) != 0).all() and not np.array_equal(m['order'], np.arange(m['m']))
    # two-id ranges give 127, 128, 129 .. 513 runs: several workgroups, the last one partly filled
    assert counts[4] + counts[5] == 511 and counts[5] + counts[6] == 513


def test_expand_between_sorts_long_runs_between_singles():
    ((seg, band, null, S, tile), p) = C.expand_between()
    m = C.run_model(seg, band, null, tile, S)
    starts = C.run_ranges(m, S)
    assert np.diff(starts)[1:4].tolist() == [288, 96, 288] == [p['runs'][i] for i in (1, 2, 3)]
    assert (m['slens'][starts[1]:starts[2]] == 1).all() and (m['slens'][starts[2]:starts[3]] == 64).all()
    assert (m['slens'][starts[3]:starts[4]] == 1).all()
    w = m['slens'][256:320]                                  # one wavefront holds the last singles of id 1 and long runs
    assert set(w.tolist()) == {1, 64} and w.sum() > 64 * 20


# ---- ids ---------------------------------------------------------------------------------------------------------
def test_id_cases():
    ((seg, band, null, S, tile), p) = C.ids_above_max()
    m = C.run_model(seg, band, null, tile, S)
    assert set(p['ignored']) <= set(np.unique(seg).tolist()) and m['ids'].max() == S == 5
    assert m['npts'] < int(((seg != 0) & (band != null)).sum())
    ((seg, band, null, S, tile), p) = C.ids_single()
    assert S == 1 and set(np.unique(seg).tolist()) == {0, 1}
    ((seg, band, null, S, tile), p) = C.ids_sparse_large()
    assert S == 1 << 20 and set(np.unique(seg).tolist()) == {0} | set(p['present'].tolist()) and len(p['present']) == 5
    assert seg.max() == S and seg[seg > 0].min() == 1
    ((seg, band, null, S, tile), p) = C.ids_gaps()
    m = C.run_model(seg, band, null, tile, S)
    assert sorted(set(m['ids'].tolist())) == [3, 4, 10] and S == 12 and (seg == 7).any()
    for kind in ('zero', 'nodata', 'norows', 'nocols'):
        ((seg, band, null, S, tile), p) = C.empty(kind)
        m = C.run_model(seg, band, null, tile, S)
        assert m['m'] == 0 and m['npts'] == 0 and m['n'] == p['n'] == seg.size
    assert C.empty('norows')[0][0].shape == (0, 70) and C.empty('nocols')[0][0].shape == (7, 0)
    assert (C.empty('nodata')[0][0] != 0).all()


# ---- values ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', C.DTYPES)
def test_value_cases_hold_every_limit(dtype):
    info = np.iinfo(dtype)
    vals = C.edge_values(dtype)
    assert {info.min, info.min + 1, info.max - 1, info.max, 0, 1} <= set(vals)
    if dtype == np.int32:
        assert {-1, -2 ** 31} <= set(vals)
    if dtype == np.uint32:
        assert {2 ** 31, 2 ** 32 - 1} <= set(vals)
    nulls = C.value_nulls(dtype)
    assert nulls[:2] == [info.min, info.max] and all(not info.min <= v <= info.max for v in nulls[2:])
    if info.min == 0:
        assert -1 in nulls
    if info.bits == 16:
        assert 70000 in nulls
    if dtype == np.uint32:
        assert 2 ** 32 in nulls
    for stripes in (False, True):
        for null in nulls:
            ((seg, band, nv, S, tile), p) = C.values(dtype, null, stripes)
            assert band.dtype == dtype and set(np.unique(band).tolist()) == set(vals)
            pts = C.visit_points(seg, band, nv, tile, S)
            labelled = int((seg != 0).sum())
            if info.min <= null <= info.max:
                assert 0 < len(pts[0]) < labelled and null not in pts[3]
            else:
                assert len(pts[0]) == labelled                  # outside the range nothing is nodata
            assert set(pts[3].tolist()) == set(vals) - {null}   # every value reaches a point, as itself
        assert seg.shape == (5, 67) and 67 % tile == 3
    ((seg, _b, _n, S, _t), _p) = C.values(dtype, 0, True)
    assert all((seg == seg[0]).all(axis=0)) and S == 6          # stripes: every id on every row


# ---- row shards --------------------------------------------------------------------------------------------------
def test_slice_cuts_reach_every_first_band_height():
    geoms = {}
    for (name, cuts) in C.SLICE_CUTS.items():
        for (lo, hi) in cuts:
            if hi > lo:
                geoms.setdefault(name, []).append((hi - lo,) + C.slice_geom(lo, hi - lo, C.SLICE_ROWS, 8))
    # (nrows, th, h0)
    assert all(h0 == 8 for (_n, _th, h0) in geoms['band-edge'])                       # h0 == th
    assert geoms['row-after'][1][2] == 7 and geoms['row-before'][1][2] == 1           # th - 1 and 1
    assert geoms['inside-one-band'][1] == (3, 8, 3)                                   # h0 == nrows, inside one band
    assert 18 // 8 == 20 // 8
    assert geoms['one-row'][1] == (1, 8, 1)
    for (name, at) in (('empty-first', 0), ('empty-middle', 1), ('empty-last', 2)):
        assert C.SLICE_CUTS[name][at] == (0, 0) and len(C.SLICE_CUTS[name]) == 3
    for cuts in C.SLICE_CUTS.values():
        rows = sorted(c for c in cuts if c[1] > c[0])
        assert rows[0][0] == 0 and rows[-1][1] == C.SLICE_ROWS and all(a[1] == b[0] for (a, b) in zip(rows, rows[1:]))
    # tile 1: every row its own band; tile 64: one band, every slice with h0 == nrows
    assert C.slice_geom(17, 23, 40, 1) == (1, 1) and C.slice_geom(17, 23, 40, 64) == (40, 23)
    assert C.SLICE_TILES == (8, 1, 64, 16) and C.SLICE_ROWS % 16 == 8        # tile 16: a short last band


@pytest.mark.parametrize('cols,tile', [(70, 8), (70, 1), (70, 64), (70, 16), (129, 128)])
def test_slice_raster_has_straddlers_and_complete_ids_under_every_cut(cols, tile):
    ((seg, band, null, S, _t), _p) = C.slice_raster(cols)
    assert seg.shape == (40, cols) and cols - (cols - 1) // min(tile, cols) * min(tile, cols) in (6, 1)
    whole = C.visit_points(seg, band, null, tile, S)
    assert _same_points(whole, H.visit_points(seg, band, null, tile, S))
    for cuts in C.SLICE_CUTS.values():
        held = [set(np.unique(seg[a:b]).tolist()) - {0} for (a, b) in cuts]
        strad = set()
        for i in range(len(held)):
            for j in range(i + 1, len(held)):
                strad |= held[i] & held[j]
        # (a rank of fewer rows than a block's four holds straddlers only)
        assert len(strad) >= 6 and all(len(h - strad) >= 3 for (h, (a, b)) in zip(held, cuts) if b - a > 4)
        # the slices' points, merged by visit index, are the whole raster's
        parts = [C.visit_points(seg[a:b], band[a:b], null, tile, S, row0=a, img_rows=40, with_key=True)
                 for (a, b) in cuts]
        cat = [np.concatenate([p[k] for p in parts]) for k in range(5)]
        order = np.lexsort((cat[4], cat[0]))
        assert _same_points(tuple(c[order] for c in cat[:4]), whole)


def test_record_cases():
    ((seg, band, null, S, tile), p) = C.records_one_id()
    assert seg.shape == (40, 300) and p['records'] == seg.size == 12000 > C.SCAN_BLOCK
    for cuts in ([(0, 20), (20, 40)], [(0, 13), (13, 27), (27, 40)]):
        ms = [C.run_model(seg[a:b], band[a:b], null, tile, S, row0=a, img_rows=40) for (a, b) in cuts]
        assert sum(m['npts'] for m in ms) == 12000 and all((m['lens'] == 64).sum() > 40 for m in ms)
    ((seg, band, null, S, tile), p) = C.records_stripes()
    assert all((seg == seg[0]).all(axis=0)) and set(np.unique(seg).tolist()) == set(range(1, S + 1))
    ((seg, band, null, S, tile), p) = C.records_bands()
    held = [set(np.unique(seg[a:b]).tolist()) for (a, b) in p['cuts']]
    assert not held[0] & held[1] and held[0] | held[1] == set(range(1, S + 1))
    ((seg, band, null, S, tile), p) = C.records_alternating()
    hist = np.bincount(seg.ravel(), minlength=S + 1)
    (a, b) = p['cuts'][0]
    m = C.run_model(seg[a:b], band[a:b], null, tile, S, row0=a, img_rows=40)
    local = np.bincount(seg[a:b].ravel(), minlength=S + 1)
    complete = (local == hist)[m['sids']]
    # inside every full wavefront of rank 0's sorted runs: complete and straddler runs alternate at least twice
    for w in range(m['m'] // 64):
        assert np.count_nonzero(np.diff(complete[w * 64:(w + 1) * 64].astype(int))) >= 2, w
    assert m['m'] // 64 >= 40 and 0 < complete.sum() < m['m']


@pytest.mark.parametrize('world,S', C.SHARE_CASES)
def test_share_cases(world, S):
    ((seg, band, null, S_, tile), p) = C.shares(world, S)
    assert S_ == S and len(p['cuts']) == world
    ranges = [C.id_range(r, world, S) for r in range(world)]
    assert ranges[0][0] == 0 and ranges[-1][1] == S + 1 and all(a[1] == b[0] for (a, b) in zip(ranges, ranges[1:]))
    held = [set(np.unique(seg[a:b]).tolist()) - {0} for (a, b) in p['cuts']]
    everywhere = set.intersection(*held)
    for (lo, hi) in ranges:
        for i in {lo, hi - 1} - {0} if hi > lo else ():
            assert i in everywhere, i                       # a straddler at id_lo and at id_hi - 1 of every share
    assert everywhere == set(p['straddlers'])
    for i in set(range(1, S + 1)) - everywhere:             # every other id is complete on rank 0
        assert i in held[0] and not any(i in h for h in held[1:])
    sizes = p['share_sizes']
    if (world, S) == (3, 9):
        assert sizes == [3, 3, 4]                           # uneven
    if (world, S) == (4, 3):
        assert sizes == [1, 1, 1, 1] and ranges[0] == (0, 1)        # one id each; rank 0's holds no segment
    if (world, S) == (4, 2):
        assert sizes == [0, 1, 1, 1] and ranges[0] == (0, 0)        # an empty share
    if (world, S) == (3, 12):
        assert sizes == [4, 4, 5] and len(everywhere) < S


def test_id_range_is_the_package_s():
    from pyshepseg_amd import distdev
    for world in (1, 2, 3, 4, 7):
        for S in (0, 1, 2, 3, 9, 12, 1000):
            for r in range(world):
                assert C.id_range(r, world, S) == distdev.idRange(r, world, S)


# ---- visit indices of 2^32 and above -----------------------------------------------------------------------------
def test_big_visit_arithmetic():
    B = C.BIG
    (R, NC, T) = (B['img_rows'], B['ncols'], B['tile'])
    assert (R, NC, T) == (65536, 65537, 8) and B['rows'] == ((65528, 65532), (65532, 65536))
    key = lambda y, x: int(C.visit_key(y, x, R, NC, T))     # noqa: E731
    # the last band starts below 2^32 and ends above it
    assert key(65528, 0) == B['band_start'] == 4294508536 < 2 ** 32 < key(65535, NC - 1) == R * NC - 1
    # the tile column at x0 = 57344 crosses 2^32 at its ninth pixel
    assert B['x0'] % T == 0 and key(65528, B['x0']) == 2 ** 32 - 8 and key(65528, B['x0'] + 7) == 2 ** 32 - 1
    assert key(65529, B['x0']) == 2 ** 32
    # the last tile column is one pixel wide
    assert (NC - 1) % T == 0 and key(65529, NC - 1) == key(65528, NC - 1) + 1
    (shards, hist) = C.big_visit_shards()
    assert [s[2] for s in shards] == [65528, 65532] and all(s[0].shape == (4, NC) for s in shards)
    assert all(s[0].nbytes <= 1 << 20 | 64 for s in shards) and hist.tolist() == [0, 128, 63, 27]
    pts = [C.visit_points(s, b, 0, T, 3, row0=lo, img_rows=R, with_key=True) for (s, b, lo) in shards]
    for (r, (p, (s, b, lo))) in enumerate(zip(pts, shards)):
        local = np.bincount(s.ravel(), minlength=4)
        assert 0 < local[1] < hist[1] and local[2 + r] == hist[2 + r] and local[3 - r] == 0
    k1 = [p[4][p[0] == 1] for p in pts]
    # both ranks hold records of id 1 on both sides of 2^32, and they interleave
    for k in k1:
        assert (k < 2 ** 32).any() and (k >= 2 ** 32).any()
    assert k1[0].min() < k1[1].min() < k1[0].max() < k1[1].max()
    # sorted by the low word alone, the order would start past 2^32
    both = np.concatenate(k1)
    assert np.sort(both & 0xFFFFFFFF)[0] == 0 and both[np.argsort(both & 0xFFFFFFFF, kind='stable')][0] == 2 ** 32
    assert len(both) == 120                                   # 128 pixels, 8 of them nodata
    # id 3 reaches into the one-pixel tile column
    assert (pts[1][1][pts[1][0] == 3] == NC - 1).sum() == 3
